"""The gate/up W4A8 grouped GEMM with fused activation and MXFP8 output (grouped_matmul_mxf8_mxf4_silu_mxf8_tn / ..._swiglu_oai_mxf8_tn) on the host: the C entry's
declaration, its rejections and the Python ops', the form rule and grid of the debug plan entry, the fake kernel and the trace of the five-launch chain's middle.
No GPU needed; the GPU half is tests/test_gpu_grouped_w4a8_act.py."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ENTRY = "qutlass_amd_grouped_matmul_mxf8_mxf4_act_mxf8_tn"
PLAN = "qutlass_amd_debug_grouped_mxf8_mxf4_act_plan"
E4, E8M0 = torch.float8_e4m3fn, torch.float8_e8m0fnu


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    L = _lib.load()
    getattr(L, PLAN).argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]   # (restype: ctypes' default, int)
    return L


def test_entry_is_declared_exported_and_bound(lib):
    from qutlass_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "qutlass_amd.h")).read()
    decl = re.search(r"\b" + ENTRY + r"\s*\(([^)]*)\)", hdr)
    assert decl is not None and len(decl.group(1).split(",")) == 18 == len(_lib.SYMBOLS[ENTRY][1])
    assert not re.search(r"\b" + PLAN + r"\b", hdr), "debug entries stay out of the public header"
    assert hasattr(lib, ENTRY) and hasattr(lib, PLAN)
    assert all(hasattr(ctypes.CDLL(build.BENCH_OUT), n) for n in (ENTRY, PLAN)), "the lab library exports both too"


@pytest.mark.parametrize("change,message", [(dict(N=96), "multiple of 64"), (dict(K=192), "K must be a positive multiple of 128"), (dict(E=1025), r"E must be in \[1, 1024\]"),
                                            (dict(act=2), "invalid act 2"), (dict(limit=7.01), "exactly representable in bf16"), (dict(bias=0x1008), "bias must be 16-byte aligned"),
                                            (dict(act=0, bias=0x1000), "takes no bias"), (dict(M=1 << 22, N=1 << 16, E=1), "2\\^24 workgroups"), (dict(), None)])
def test_c_entry_rejections(lib, change, message):
    a = {**dict(act=1, limit=7.0, bias=None, M=0, N=128, K=256, E=4), **change}
    d = ctypes.c_void_p(0x1000)   # never dereferenced: every call here returns before a launch (the accepted one through M == 0)
    rc = getattr(lib, ENTRY)(d, d, d, d, d, 1, d, a["act"], 1.702, a["limit"], a["bias"], d, d, a["M"], a["N"], a["K"], a["E"], None)
    assert (rc == 0) if message is None else (rc == 1 and re.search(message, lib.qutlass_amd_last_error().decode())), lib.qutlass_amd_last_error().decode()


@pytest.mark.parametrize("M,inter,K,E", [(16, 2944, 2944, 32), (64, 768, 2048, 128), (4096, 768, 2048, 128), (16384, 2944, 2944, 32), (8192, 14336, 4096, 8),
                                         (128, 32, 1024, 4), (128, 32, 1152, 4), (127, 32, 1152, 4), (0, 64, 128, 1)])
def test_plan_rule_and_grid(lib, M, inter, K, E):
    """the committed rule: mean rows per group >= 32 and K > 1024 -> 615, else 614; the grid counts tiles of 32 ACTIVATION columns"""
    out = (ctypes.c_int64 * 1)(-1)
    v = getattr(lib, PLAN)(M, 2 * inter, K, E, out)
    assert v == (615 if M >= 32 * E and K > 1024 else 614)
    assert out[0] == (0 if M == 0 else ((M + (v - 613) * 32 - 1) // ((v - 613) * 32) + E) * (inter // 32))   # TM = 32 (614), 64 (615)
    assert getattr(lib, PLAN)(M, 2 * inter + 32, K, E, out) == -1, "N % 64"


def _operands(M=48, inter=64, K=256, E=4, adtype=E4):
    return [torch.zeros(M, K, dtype=torch.uint8).view(adtype), torch.zeros(E, 2 * inter, K // 2, dtype=torch.uint8), torch.zeros(M * K // 32, dtype=torch.uint8).view(E8M0),
            torch.zeros(E * 2 * inter * K // 32, dtype=torch.uint8).view(E8M0), torch.ones(1), torch.full((E,), M, dtype=torch.int32)]


def test_python_rejections_come_before_any_device_work():
    """CPU tensors on a machine that may have no GPU: each call raises its own message, so nothing was dispatched"""
    import qutlass
    import qutlass_amd as q

    silu, oai = q.grouped_matmul_mxf8_mxf4_silu_mxf8_tn, q.grouped_matmul_mxf8_mxf4_swiglu_oai_mxf8_tn
    assert qutlass.grouped_matmul_mxf8_mxf4_silu_mxf8_tn is silu and qutlass.grouped_matmul_mxf8_mxf4_swiglu_oai_mxf8_tn is oai
    for f in (silu, oai):
        assert f.__doc__.startswith("EXTENSION") and "grouped_matmul_mxf8_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs)" in f.__doc__ and f.__name__ in q.__doc__
        for kw, message in ((dict(adtype=torch.float8_e5m2), f.__name__ + ": a must be float8_e4m3fn, float8_e5m2 tokens are not supported"),
                            (dict(inter=48), "I a multiple of 32"), (dict(K=192), r"K must be a multiple of 128 \(got 192\)"),
                            (dict(M=1, inter=32, K=128, E=1025), r"experts must be in \[1, 1024\] \(got 1025\)")):
            with pytest.raises(ValueError, match=message):
                f(*_operands(**kw))
    for kw, message in ((dict(bias=torch.zeros(4, 64, dtype=torch.bfloat16)), r"bias must be \(E, 2 \* I\) = \(4, 128\)"), (dict(bias=torch.zeros(4, 128)), "bias must be bfloat16"),
                        (dict(limit=7.01), "limit must be > 0, finite and exactly representable in bf16"), (dict(act_alpha=float("nan")), "act_alpha must be finite and > 0")):
        with pytest.raises(ValueError, match=message):
            oai(*_operands(), **kw)


def test_fake_kernel_and_chain_trace():
    """gather-quantise -> this op -> down GEMM: three ops in the trace and nothing that reads a tensor's value on the host"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.proxy_tensor import make_fx

    import qutlass_amd as q

    q.ops.register_torch_ops()
    assert torch._library.simple_registry.singleton.find("qutlass_amd::grouped_matmul_mxf8_mxf4_act_mxf8").fake_impl.kernel is not None
    T, M, inter, K, E = 40, 160, 96, 256, 4

    def layer(x, h, src_row, w13, w13_sf, w2, w2_sf, bias, alpha, offs):
        a, a_sf = q.fusedGatherQuantizeMxf8(x, h, src_row)
        c, c_sf = q.grouped_matmul_mxf8_mxf4_swiglu_oai_mxf8_tn(a, w13, a_sf, w13_sf, alpha, offs, bias=bias)
        return c, c_sf, q.grouped_matmul_mxf8_mxf4_bf16_tn(c, w2, c_sf, w2_sf, alpha, offs)

    with FakeTensorMode():
        args = (torch.empty(T, K, dtype=torch.bfloat16, device=DEV), torch.empty(32, 32, dtype=torch.bfloat16, device=DEV), torch.empty(M, dtype=torch.int32, device=DEV),
                torch.empty(E, 2 * inter, K // 2, dtype=torch.uint8, device=DEV), torch.empty(E * 2 * inter * K // 32, dtype=E8M0, device=DEV),
                torch.empty(E, K, inter // 2, dtype=torch.uint8, device=DEV), torch.empty(E * K * inter // 32, dtype=E8M0, device=DEV),
                torch.empty(E, 2 * inter, dtype=torch.bfloat16, device=DEV), torch.empty(E, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV))
        c, c_sf, y = layer(*args)
        assert tuple(c.shape) == (M, inter) and c.dtype == E4 and tuple(c_sf.shape) == (256, 4) and c_sf.dtype == E8M0 and tuple(y.shape) == (M, K)
        gm = make_fx(layer, tracing_mode="fake")(*args)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert "qutlass_amd.grouped_matmul_mxf8_mxf4_act_mxf8.default" in targets and "qutlass_amd.grouped_matmul_mxf8_mxf4.default" in targets, targets
    assert any("ather" in t and "xf8" in t for t in targets), targets
    assert not any(s in t for t in targets for s in ("aten.item", "_local_scalar_dense", "nonzero", "_to_copy")), targets
