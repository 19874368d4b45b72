"""Grouped MXFP4 GEMM (grouped_matmul_mxf4_bf16_tn, csrc/gemm_mx_grouped.hip.h) on the host: the C entry's argument checks, the tile decode the device runs (through
qutlass_amd_debug_grouped_decode, the same lane functions compiled for the host), the form rule, and the torch op's fake kernel.  No GPU needed; the GPU half is
tests/test_gpu_grouped.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    L = _lib.load()
    L.qutlass_amd_debug_grouped_decode.restype = ctypes.c_int
    L.qutlass_amd_debug_grouped_decode.argtypes = [ctypes.POINTER(ctypes.c_int32)] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    L.qutlass_amd_debug_grouped_plan.restype = ctypes.c_int
    L.qutlass_amd_debug_grouped_plan.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    return L


def test_entry_is_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "qutlass_amd.h")).read()
    assert re.search(r"\bqutlass_amd_grouped_matmul_mxf4_bf16_tn\s*\(", hdr)
    assert hasattr(lib, "qutlass_amd_grouped_matmul_mxf4_bf16_tn")
    from qutlass_amd._lib import SYMBOLS

    assert "qutlass_amd_grouped_matmul_mxf4_bf16_tn" in SYMBOLS


def test_entry_rejects_bad_arguments_without_launching(lib):
    from qutlass_amd._lib import QAMD_ERR_INVALID

    d = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first
    g = lib.qutlass_amd_grouped_matmul_mxf4_bf16_tn
    err = lambda: lib.qutlass_amd_last_error().decode()

    def call(A=d, B=d, A_sf=d, B_sf=d, alpha=d, n_alpha=1, offs=d, D=d, M=64, N=256, K=512, E=8):
        return g(A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E, None)

    for k in ("A", "B", "A_sf", "B_sf", "alpha", "offs", "D"):
        assert call(**{k: None}) == QAMD_ERR_INVALID, k
        assert "null pointer" in err()
    for E in (0, -1, 1025):
        assert call(E=E) == QAMD_ERR_INVALID and "E must be in [1, 1024]" in err(), E
    assert call(K=96) == QAMD_ERR_INVALID and "multiple of 128" in err()
    assert call(K=640 + 64) == QAMD_ERR_INVALID and "multiple of 128" in err()
    assert call(N=260) == QAMD_ERR_INVALID and "multiple of 8" in err()
    assert call(n_alpha=3) == QAMD_ERR_INVALID and "alpha" in err()
    assert call(N=16384, K=262144) == QAMD_ERR_INVALID and "below 2 GiB" in err()        # one expert of exactly 2 GiB
    assert call(M=-1) == QAMD_ERR_INVALID
    assert call(M=1 << 24, K=256) == QAMD_ERR_INVALID and "token matrix" in err()
    # M == 0: accepted, nothing launched (this machine may have no GPU at all)
    assert call(M=0) == 0


def _decode(lib, offs, M, TM, tiles_n):
    offs = np.ascontiguousarray(offs, dtype=np.int32)
    E = len(offs)
    nwg = (-(-M // TM) + E) * tiles_n         # the host's grid bound
    out = (ctypes.c_int * (4 * nwg))()
    n = lib.qutlass_amd_debug_grouped_decode(offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), E, M, TM, tiles_n, nwg, out)
    return n, np.frombuffer(out, dtype=np.int32).reshape(nwg, 4).copy()


def _coverage(t, n, M, TM, tiles_n, E):
    """rows covered per column tile; the real workgroups are the first n, every (tile, column tile) once"""
    assert (t[:n, 0] >= 0).all() and (t[n:, 0] == -1).all(), "the workgroups without work are the last ones"
    real = t[:n]
    assert len({(g, r0, nt) for g, r0, _, nt in real}) == n
    cover = np.zeros((tiles_n, M), dtype=np.int64)
    for g, r0, rows, nt in real:
        assert 0 <= g < E and 1 <= rows <= TM and 0 <= r0 and r0 + rows <= M and 0 <= nt < tiles_n, (g, r0, rows, nt)
        cover[nt, r0:r0 + rows] += 1
    return real, cover


def _check_wellformed(lib, offs, M, TM, tiles_n=3):
    offs = np.asarray(offs, dtype=np.int64)
    E = len(offs)
    n, t = _decode(lib, offs, M, TM, tiles_n)
    starts = np.concatenate([[0], offs[:-1]])
    assert n == tiles_n * sum(-(-(e - s) // TM) for s, e in zip(starts, offs))   # ceil(rows_g / TM) tiles per group and column tile
    real, cover = _coverage(t, n, M, TM, tiles_n, E)
    for g, r0, rows, nt in real:
        assert starts[g] <= r0 and r0 + rows <= offs[g], (g, r0, rows)              # inside its group
    end = int(offs[-1])
    assert (cover[:, :end] == 1).all(), "every row of [0, offs[-1]) exactly once per column tile"
    assert (cover[:, end:] == 0).all(), "rows past offs[-1] are not covered"


def _route(rng, M, E, kind):
    if kind == "uniform":
        counts = np.bincount(rng.integers(0, E, M), minlength=E)
    elif kind == "skewed":           # half of the rows in one expert
        counts = np.bincount(rng.integers(0, E, M - M // 2), minlength=E)
        counts[rng.integers(0, E)] += M // 2
    elif kind == "empty":            # most experts get nothing
        live = rng.choice(E, size=max(1, E // 8), replace=False)
        counts = np.zeros(E, dtype=np.int64)
        counts[live] = np.bincount(rng.integers(0, len(live), M), minlength=len(live))
    return np.cumsum(counts)


@pytest.mark.parametrize("TM", [32, 64])
def test_decode_covers_every_row_once(lib, TM):
    rng = np.random.default_rng(7)
    for E in (1, 2, 8, 63, 64, 65, 128, 256, 1000, 1024):
        for M in (1, 31, 64, 512, 4099):
            for kind in ("uniform", "skewed", "empty"):
                _check_wellformed(lib, _route(rng, M, E, kind), M, TM)
    _check_wellformed(lib, [4096], 4096, TM)                               # E = 1
    _check_wellformed(lib, _route(rng, 700, 16, "skewed"), 700, TM, tiles_n=1)
    _check_wellformed(lib, _route(rng, 700, 16, "uniform"), 700, TM, tiles_n=48)
    _check_wellformed(lib, [0] * 7 + [300], 300, TM)                         # everything in the last expert
    _check_wellformed(lib, [300] * 8, 300, TM)                               # everything in the first
    _check_wellformed(lib, [0] * 16, 64, TM)                                 # all empty
    offs = _route(rng, 1000, 128, "uniform")
    _check_wellformed(lib, np.minimum(offs, 700), 1000, TM)                 # offs[-1] < M: rows 700 ... 999 untouched


def test_decode_of_malformed_offsets_stays_inside_m(lib):
    rng = np.random.default_rng(3)
    M = 517
    cases = [[600, 10, 20, 700], [-5, 40, 30, 1 << 30], [M + 1] * 4, [-(1 << 31)] * 3 + [2 ** 31 - 1], [300, 200, 100], [10, -10, 20]]
    for _ in range(100):
        E = int(rng.integers(1, 300))
        cases.append(rng.integers(-100, M + 200, E))
    for offs in cases:
        for TM in (32, 64):
            E = len(offs)
            n, t = _decode(lib, offs, M, TM, 2)      # (every workgroup index of the grid bound: the decode never goes past it)
            real, cover = _coverage(t, n, M, TM, 2, E)
            assert (cover <= 1).all(), "no row written twice"
            # the clamped running maximum: group g covers [max(clamp(offs[:g])), max(clamp(offs[:g+1])))
            ends = np.maximum.accumulate(np.clip(np.asarray(offs, dtype=np.int64), 0, M))
            assert (cover[:, :ends[-1]] == 1).all() and (cover[:, ends[-1]:] == 0).all()


def test_plan_follows_the_documented_rule(lib):
    p = lib.qutlass_amd_debug_grouped_plan
    grid = ctypes.c_int64()
    for E in (1, 8, 128, 256):
        for M in (1, 16 * E, 32 * E, 32 * E + 1, 64 * E, 64 * E + 1, 4096 * 8):
            for K in (256, 768, 1024, 1152, 2048, 4096, 14336):
                v = p(M, 2048, K, E, ctypes.byref(grid))
                want = 590 if M <= 32 * E and K <= 1024 else 593      # mean rows per group and K
                assert v == want, (M, K, E, v)
                TM, TN = {590: (32, 32), 593: (64, 64)}[v]
                assert grid.value == (-(-M // TM) + E) * (2048 // TN)
    assert p(0, 2048, 768, 8, None) == 590
    assert p(64, 2048, 4000, 8, None) == -1       # K % 128
    assert p(64, 2044, 4096, 8, None) == -1       # N % 8
    assert p(64, 2048, 4096, 0, None) == -1       # E
    assert p(64, 2048, 4096, 1025, None) == -1


def test_fake_kernel_and_aot_graph():
    from torch._dynamo.backends.common import aot_autograd
    from torch._subclasses.fake_tensor import FakeTensorMode

    import qutlass  # the drop-in alias reaches the extension too
    import qutlass_amd as q

    assert qutlass.grouped_matmul_mxf4_bf16_tn is q.grouped_matmul_mxf4_bf16_tn
    assert q.grouped_matmul_mxf4_bf16_tn.__doc__.startswith("EXTENSION")
    q.ops.register_torch_ops()
    assert torch._library.simple_registry.singleton.find("qutlass_amd::grouped_matmul_mxf4").fake_impl.kernel is not None
    M, N, K, E = 96, 256, 512, 4
    with FakeTensorMode():
        a = torch.empty(M, K // 2, dtype=torch.uint8, device=DEV)
        b = torch.empty(E, N, K // 2, dtype=torch.uint8, device=DEV)
        a_sf = torch.empty(M * K // 32, dtype=torch.float8_e8m0fnu, device=DEV)
        b_sf = torch.empty(E * N * K // 32, dtype=torch.float8_e8m0fnu, device=DEV)
        alpha = torch.empty(E, device=DEV)
        offs = torch.empty(E, dtype=torch.int32, device=DEV)
        out = q.grouped_matmul_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs)
        assert out.shape == (M, N) and out.dtype == torch.bfloat16 and out.device.type == "cuda"

    graphs = []

    def capture(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def layer(a, b, a_sf, b_sf, alpha, offs):
        return q.grouped_matmul_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs) * 2

    torch._dynamo.reset()
    args = (torch.zeros(M, K // 2, dtype=torch.uint8), torch.zeros(E, N, K // 2, dtype=torch.uint8),
            torch.zeros(M * K // 32, dtype=torch.uint8).view(torch.float8_e8m0fnu), torch.zeros(E * N * K // 32, dtype=torch.uint8).view(torch.float8_e8m0fnu),
            torch.ones(1), torch.full((E,), M, dtype=torch.int32))
    try:   # CPU tensors: tracing never looks at the device, and the run after it has no kernel to call (CUDA key only) -- the graph exists by then
        torch.compile(layer, backend=aot_autograd(fw_compiler=capture), fullgraph=True)(*args)
    except (NotImplementedError, RuntimeError) as e:
        assert graphs and ("CPU" in str(e) or "backend" in str(e)), e
    assert graphs
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert "qutlass_amd.grouped_matmul_mxf4.default" in targets, targets
