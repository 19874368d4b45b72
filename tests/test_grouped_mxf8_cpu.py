"""Grouped MXFP8 GEMM (grouped_matmul_mxf8_bf16_tn) on the host: the C entry's declaration and argument checks, the form rule (through
qutlass_amd_debug_grouped_mxf8_plan), and the torch op's fake kernel.  The tile decode is the MXFP4 op's (tests/test_grouped_cpu.py).  No GPU needed; the GPU
half is tests/test_gpu_grouped_mxf8.py."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ENTRY = "qutlass_amd_grouped_matmul_mxf8_bf16_tn"


def _bench_lib_path():
    from qutlass_amd import build

    return build.BENCH_OUT


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    L = _lib.load()
    L.qutlass_amd_debug_grouped_mxf8_plan.restype = ctypes.c_int
    L.qutlass_amd_debug_grouped_mxf8_plan.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    return L


def test_entry_is_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "qutlass_amd.h")).read()
    assert re.search(r"\bqutlass_amd_grouped_matmul_mxf8_bf16_tn\s*\(", hdr)
    assert not re.search(r"\bqutlass_amd_debug_grouped_mxf8_plan\b", hdr), "debug entries stay out of the public header"
    assert hasattr(lib, ENTRY)
    from qutlass_amd._lib import SYMBOLS

    assert ENTRY in SYMBOLS
    path = _bench_lib_path()
    assert os.path.exists(path), path
    assert hasattr(ctypes.CDLL(path), ENTRY), "the lab library exports the entry too"


def test_entry_rejects_bad_arguments_without_launching(lib):
    from qutlass_amd._lib import QAMD_ERR_INVALID

    d = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first
    g = getattr(lib, ENTRY)
    err = lambda: lib.qutlass_amd_last_error().decode()

    def call(A=d, B=d, A_sf=d, B_sf=d, alpha=d, n_alpha=1, offs=d, D=d, M=64, N=256, K=512, E=8, a_format=0):
        return g(A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E, a_format, None)

    for k in ("A", "B", "A_sf", "B_sf", "alpha", "offs", "D"):
        assert call(**{k: None}) == QAMD_ERR_INVALID, k
        assert "null pointer" in err()
    for E in (0, -1, 1025):
        assert call(E=E) == QAMD_ERR_INVALID and "E must be in [1, 1024]" in err(), E
    for n_alpha in (0, 3, 9):
        assert call(n_alpha=n_alpha) == QAMD_ERR_INVALID and "alpha" in err(), n_alpha
    assert call(K=96) == QAMD_ERR_INVALID and "multiple of 128" in err()
    assert call(K=640 + 64) == QAMD_ERR_INVALID and "multiple of 128" in err()
    assert call(N=260) == QAMD_ERR_INVALID and "multiple of 8" in err()
    for fmt in (2, -1):
        assert call(a_format=fmt) == QAMD_ERR_INVALID and "a_format" in err(), fmt
    # one expert of N * K = 2^31 bytes: below the MXFP4 entry's N * K/2 bound, rejected here
    assert call(N=16384, K=131072) == QAMD_ERR_INVALID and "below 2 GiB" in err()
    assert call(M=16384, N=256, K=131072) == QAMD_ERR_INVALID and "below 2 GiB" in err()   # token matrix of 2^31 bytes
    assert call(M=1 << 24, K=128) == QAMD_ERR_INVALID and "token matrix" in err()
    assert call(M=-1) == QAMD_ERR_INVALID
    # M == 0: accepted, nothing launched (this machine may have no GPU at all) -- both A formats, per-expert alpha
    assert call(M=0) == 0
    assert call(M=0, a_format=1, n_alpha=8) == 0
    # just below the limits
    assert call(M=0, N=16376, K=131072) == 0


def _want(M, K, E):
    return 594 if M <= 32 * E and K >= 8192 else 597   # mean rows per group and K


def test_plan_follows_the_documented_rule(lib):
    p = lib.qutlass_amd_debug_grouped_mxf8_plan
    grid = ctypes.c_int64()
    shapes = [   # (E, N, K): Qwen3-30B-A3B and Mixtral-8x7B gate/up and down, plus edges
        (128, 1536, 2048), (128, 2048, 768), (8, 28672, 4096), (8, 4096, 14336), (1, 2048, 8192), (256, 512, 8064), (64, 1024, 16384),
    ]
    for E, N, K in shapes:
        for M in (1, 16 * E, 32 * E, 32 * E + 1, 64 * E, 4096 * 8):   # decode and prefill
            v = p(M, N, K, E, ctypes.byref(grid))
            assert v == _want(M, K, E), (M, N, K, E, v)
            TM, TN = {594: (32, 32), 597: (64, 64)}[v]
            assert grid.value == (-(-M // TM) + E) * (-(-N // TN)), (M, N, K, E)
    assert p(128, 4096, 14336, 8, None) == 594        # Mixtral down decode: 16 rows per expert
    assert p(8192, 4096, 14336, 8, None) == 597       # ... prefill
    assert p(512, 2048, 768, 128, None) == 597        # Qwen3 down decode: a short K stays with the ring form (MXFP4: 590)
    assert p(0, 2048, 8192, 8, None) == 594 and p(0, 2048, 768, 8, None) == 597
    assert p(64, 2048, 4000, 8, None) == -1       # K % 128
    assert p(64, 2044, 4096, 8, None) == -1       # N % 8
    assert p(64, 2048, 4096, 0, None) == -1       # E
    assert p(64, 2048, 4096, 1025, None) == -1
    assert p(64, 16384, 131072, 8, None) == -1    # one expert of 2 GiB


@pytest.mark.parametrize("adtype", [torch.float8_e4m3fn, torch.float8_e5m2])
def test_fake_kernel_and_aot_graph(adtype):
    from torch._dynamo.backends.common import aot_autograd
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.proxy_tensor import make_fx

    import qutlass  # the drop-in alias reaches the extension too
    import qutlass_amd as q

    assert qutlass.grouped_matmul_mxf8_bf16_tn is q.grouped_matmul_mxf8_bf16_tn
    assert q.grouped_matmul_mxf8_bf16_tn.__doc__.startswith("EXTENSION")
    assert "grouped_matmul_mxf8_bf16_tn" in q.__doc__
    q.ops.register_torch_ops()
    assert torch._library.simple_registry.singleton.find("qutlass_amd::grouped_matmul_mxf8").fake_impl.kernel is not None
    M, N, K, E = 96, 256, 512, 4
    with FakeTensorMode():
        a = torch.empty(M, K, dtype=adtype, device=DEV)
        b = torch.empty(E, N, K, dtype=torch.float8_e4m3fn, device=DEV)
        a_sf = torch.empty(M * K // 32, dtype=torch.float8_e8m0fnu, device=DEV)
        b_sf = torch.empty(E * N * K // 32, dtype=torch.float8_e8m0fnu, device=DEV)
        alpha = torch.empty(E, device=DEV)
        offs = torch.empty(E, dtype=torch.int32, device=DEV)
        out = q.grouped_matmul_mxf8_bf16_tn(a, b, a_sf, b_sf, alpha, offs)
        assert out.shape == (M, N) and out.dtype == torch.bfloat16 and out.device.type == "cuda"

    def layer(a, b, a_sf, b_sf, alpha, offs):
        return q.grouped_matmul_mxf8_bf16_tn(a, b, a_sf, b_sf, alpha, offs) * 2

    args = (torch.zeros(M, K, dtype=torch.uint8).view(adtype), torch.zeros(E, N, K, dtype=torch.uint8).view(torch.float8_e4m3fn),
            torch.zeros(M * K // 32, dtype=torch.uint8).view(torch.float8_e8m0fnu), torch.zeros(E * N * K // 32, dtype=torch.uint8).view(torch.float8_e8m0fnu),
            torch.ones(1), torch.full((E,), M, dtype=torch.int32))

    gm = make_fx(layer, tracing_mode="fake")(*args)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert "qutlass_amd.grouped_matmul_mxf8.default" in targets, targets

    graphs = []

    def capture(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    torch._dynamo.reset()
    try:   # CPU tensors: tracing never looks at the device, and the run after it has no kernel to call (CUDA key only) -- the graph exists by then
        torch.compile(layer, backend=aot_autograd(fw_compiler=capture), fullgraph=True)(*args)
    except (NotImplementedError, RuntimeError) as e:
        assert graphs and ("CPU" in str(e) or "backend" in str(e)), e
    assert graphs
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert "qutlass_amd.grouped_matmul_mxf8.default" in targets, targets
