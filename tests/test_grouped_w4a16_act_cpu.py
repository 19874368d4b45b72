"""The gate/up W4A16 grouped GEMM with fused activation and bf16 output (grouped_matmul_bf16_mxf4_silu_bf16_tn / ..._swiglu_oai_bf16_tn) on the host: the C entry's
declaration, its rejections and the Python ops', the form rule and grid of the debug plan entry, and the fake kernel.  No GPU needed; the GPU half is
tests/test_gpu_grouped_w4a16_act.py."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "qutlass_amd_grouped_matmul_bf16_mxf4_act_bf16_tn"
PLAN = "qutlass_amd_debug_grouped_bf16_mxf4_act_plan"
E8M0 = torch.float8_e8m0fnu


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


@pytest.mark.parametrize("change,message", [(dict(N=96), "multiple of 64"), (dict(N=100), "N must be a multiple of 8"), (dict(K=192), "K must be a positive multiple of 128"),
                                            (dict(K=0), "K must be a positive multiple of 128"), (dict(E=1025), r"E must be in \[1, 1024\]"), (dict(E=0), r"E must be in \[1, 1024\]"),
                                            (dict(n_alpha=3), "alpha must have 1 or E"), (dict(M=-1), "M must be >= 0"), (dict(M=1 << 23, K=128), "token matrix"),
                                            (dict(N=1 << 25, K=128), "one expert's weight"), (dict(M=1 << 22, N=1 << 16, K=128, E=1), "2\\^24 workgroups"),
                                            (dict(act=2), "invalid act 2"), (dict(limit=7.01), "exactly representable in bf16"), (dict(bias=0x1008), "bias must be 16-byte aligned"),
                                            (dict(act=0, bias=0x1000), "takes no bias"), (dict(D=0x1008), "D must be 16-byte aligned"),
                                            (dict(src=0x1000, T=1 << 22, K=256), "gathered token matrix"), (dict(src=0x1000, T=-1), "T must be >= 0"),
                                            (dict(src=0x1000, T=(1 << 22) - 1, K=256), None), (dict(n_alpha=4), None), (dict(), None)])
def test_c_entry_boundaries(lib, change, message):
    a = {**dict(act=1, limit=7.0, bias=None, src=None, T=0, n_alpha=1, D=0x1000, M=0, N=128, K=256, E=4), **change}
    d = ctypes.c_void_p(0x1000)   # never dereferenced: every call here returns before a launch (the accepted ones through M == 0)
    rc = getattr(lib, ENTRY)(d, d, d, d, a["n_alpha"], d, a["src"], a["T"], a["act"], 1.702, a["limit"], a["bias"], a["D"], a["M"], a["N"], a["K"], a["E"], None)
    err = lib.qutlass_amd_last_error().decode()
    assert (rc == 0) if message is None else (rc == 1 and re.search(message, err)), err
    if "src" not in change and "act" not in change and "bias" not in change and "limit" not in change and "D" not in change and "n_alpha" not in change:
        assert (getattr(lib, PLAN)(a["M"], a["N"], a["K"], a["E"], None) == -1) == (message is not None), "the plan entry runs the entry's shape checks"


@pytest.mark.parametrize("M,inter,K,E", [(16, 2944, 2944, 32), (64, 768, 2048, 128), (4096, 768, 2048, 128), (16384, 2944, 2944, 32), (8192, 14336, 4096, 8),
                                         (1024, 32, 512, 4), (1024, 32, 640, 4), (1023, 32, 640, 4), (0, 64, 128, 1)])
def test_plan_rule_and_grid(lib, M, inter, K, E):
    """the committed rule: mean rows per group >= 256 and K > 512 -> 619, else 618; the grid counts tiles of 32 ACTIVATION columns"""
    out = (ctypes.c_int64 * 1)(-1)
    v = getattr(lib, PLAN)(M, 2 * inter, K, E, out)
    assert v == (619 if M >= 256 * E and K > 512 else 618)
    TM = 32 * (v - 617)
    assert out[0] == (0 if M == 0 else ((M + TM - 1) // TM + E) * (inter // 32))
    assert getattr(lib, PLAN)(M, 2 * inter + 32, K, E, out) == -1, "N % 64"


def test_every_form_of_the_rule_is_met(lib):
    picked = {getattr(lib, PLAN)(M, 128, K, 4, None) for M in (16, 128, 1024) for K in (128, 512, 640, 2944)}
    assert picked == {618, 619}


def _operands(M=48, inter=64, K=256, E=4, adtype=torch.bfloat16):
    return [torch.zeros(M, K, dtype=adtype), torch.zeros(E, 2 * inter, K // 2, dtype=torch.uint8), torch.zeros(E * 2 * inter * K // 32, dtype=torch.uint8).view(E8M0),
            torch.ones(1), torch.full((E,), M, dtype=torch.int32)]


def test_python_rejections_come_before_any_device_work():
    """CPU tensors on a machine that may have no GPU: each call raises its own message, so nothing was dispatched"""
    import qutlass
    import qutlass_amd as q

    silu, oai = q.grouped_matmul_bf16_mxf4_silu_bf16_tn, q.grouped_matmul_bf16_mxf4_swiglu_oai_bf16_tn
    assert qutlass.grouped_matmul_bf16_mxf4_silu_bf16_tn is silu and qutlass.grouped_matmul_bf16_mxf4_swiglu_oai_bf16_tn is oai
    for f in (silu, oai):
        assert f.__doc__.startswith("EXTENSION") and "grouped_matmul_bf16_mxf4_bf16_tn(a, b, b_sf, alpha, offs, src_row=src_row)" in f.__doc__ and f.__name__ in q.__doc__
        for kw, message in ((dict(adtype=torch.float16), f.__name__ + ": a must be bfloat16"), (dict(inter=48), "I a multiple of 32"),
                            (dict(K=192), r"K must be a multiple of 128 \(got 192\)"), (dict(M=1, inter=32, K=128, E=1025), r"experts must be in \[1, 1024\] \(got 1025\)"),
                            (dict(src_row=torch.zeros(48, dtype=torch.int64)), "src_row must be a 1D int32 tensor")):
            with pytest.raises(ValueError, match=message):
                f(*_operands(**{k: v for k, v in kw.items() if k != "src_row"}), **{k: v for k, v in kw.items() if k == "src_row"})
    for kw, message in ((dict(bias=torch.zeros(4, 64, dtype=torch.bfloat16)), r"bias must be \(E, 2 \* I\) = \(4, 128\)"), (dict(bias=torch.zeros(4, 128)), "bias must be bfloat16"),
                        (dict(limit=7.01), "limit must be > 0, finite and exactly representable in bf16"), (dict(act_alpha=float("nan")), "act_alpha must be finite and > 0")):
        with pytest.raises(ValueError, match=message):
            oai(*_operands(), **kw)


def test_fake_kernel_and_chain_trace():
    """this op with src_row -> down GEMM: two ops in the trace and nothing that reads a tensor's value on the host"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.proxy_tensor import make_fx

    import qutlass_amd as q

    q.ops.register_torch_ops()
    assert torch._library.simple_registry.singleton.find("qutlass_amd::grouped_matmul_bf16_mxf4_act_bf16").fake_impl.kernel is not None
    T, M, inter, K, E, dev = 40, 160, 96, 256, 4, "cuda"

    def layer(x, src_row, w13, w13_sf, w2, w2_sf, bias, alpha, offs):
        h = q.grouped_matmul_bf16_mxf4_swiglu_oai_bf16_tn(x, w13, w13_sf, alpha, offs, bias=bias, src_row=src_row)
        return h, q.grouped_matmul_bf16_mxf4_bf16_tn(h, w2, w2_sf, alpha, offs)

    with FakeTensorMode():
        args = (torch.empty(T, K, dtype=torch.bfloat16, device=dev), torch.empty(M, dtype=torch.int32, device=dev),
                torch.empty(E, 2 * inter, K // 2, dtype=torch.uint8, device=dev), torch.empty(E * 2 * inter * K // 32, dtype=E8M0, device=dev),
                torch.empty(E, K, inter // 2, dtype=torch.uint8, device=dev), torch.empty(E * K * inter // 32, dtype=E8M0, device=dev),
                torch.empty(E, 2 * inter, dtype=torch.bfloat16, device=dev), torch.empty(E, device=dev), torch.empty(E, dtype=torch.int32, device=dev))
        h, y = layer(*args)
        assert tuple(h.shape) == (M, inter) and h.dtype == torch.bfloat16 and tuple(y.shape) == (M, K)
        gm = make_fx(layer, tracing_mode="fake")(*args)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count("qutlass_amd.grouped_matmul_bf16_mxf4_act_bf16.default") == 1 and "qutlass_amd.grouped_matmul_bf16_mxf4_bf16_tn.default" in targets, targets
    assert not any(s in t for t in targets for s in ("aten.item", "_local_scalar_dense", "nonzero", "_to_copy")), targets
